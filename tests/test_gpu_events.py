"""-vcf on the MI355X (slamem_pileup_enable_events / _events_* / _add_events_* / _rows_at_*, engine.Pileup(events=True), the
executable): every table is tests/events_spec.py applied to the same observations, compared for exact equality -- planted events
(un-normalised inside a homopolymer, a tandem repeat and next to a separator; alleles that share a position; the longest
lengths), contention on one key and on 64 alleles of one position, a table that is too small, the skipped counters, real mappings
with indels whatever the batches' order, the stream or the number of accumulators -- and, without the spec, a known answer: a
planted deletion inside a homopolymer."""
import ctypes as C
import os
import subprocess
import threading

import numpy as np
import pytest

import events_spec as es
import sites_spec
from test_events_host import planted_deletion
from test_gpu_chain import indel_reads
from test_gpu_map import multi_record_batch
from test_gpu_pile import spec_results
from test_gpu_sites import halves, run_stream, windows, write_fasta

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "slamem_amd", "host", "slaMEM-hip")


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test without a GPU")
    from slamem_amd import engine
    return engine


def got_events(p, **kw):
    arr, skipped = p.events(**kw)
    assert arr.dtype == p_dtype() and not arr["pad"].any()
    return es.from_records(arr), skipped


def p_dtype():
    from slamem_amd import engine
    return engine.EVENT_DTYPE


# ---- planted events ------------------------------------------------------------------------------------------------------------

def planted_text():
    """5,000 letters in three records (separators at 2000 and 3500): a run of 300 A from 500, (AC) x 100 from 1000, TTTT right
    behind the first separator."""
    rng = np.random.default_rng(23)
    t = rng.choice(ACGT, size=5000)
    t[499], t[500:800], t[800] = ord("C"), ord("A"), ord("G")
    t[999] = ord("G")
    t[1000:1200] = np.frombuffer(b"AC" * 100, dtype=np.uint8)
    t[1200] = ord("T")
    t[2000] = t[3500] = ord("N")
    t[2001:2005] = ord("T")
    t[2005] = ord("G")
    t[4200:4210] = np.frombuffer(b"acgtacgtac", dtype=np.uint8)  # (lower case folds)
    return t


def plants(text):
    rng = np.random.default_rng(29)
    T = bytes(text)
    ev = [
        # one position and length, different letters; an insertion and a deletion at one position
        (3000, 1, 2, b"GA", 3, 1), (3000, 1, 2, b"GC", 1, 0), (3000, 1, 2, b"TA", 0, 2), (3000, 0, 2, b"", 2, 2), (3000, 1, 1, b"G", 5, 0),
        # the longest lengths
        (2500, 1, 31, bytes(rng.choice(ACGT, size=31)), 1, 1), (2600, 1, 31, b"A" * 31, 0, 1), (2700, 0, 127, b"", 2, 0),
        (4000, 1, 1, b"A", 1, 0), (4000, 1, 1, b"C", 1, 0), (4000, 1, 1, b"G", 1, 0), (4000, 1, 1, b"T", 1, 0),
        # un-normalised inside the run of A: all of these are one deletion and one insertion at 500
        (650, 0, 3, b"", 1, 0), (797, 0, 3, b"", 0, 1), (500, 0, 3, b"", 1, 1), (700, 1, 2, b"AA", 1, 0), (800, 1, 2, b"AA", 0, 1),
        (799, 0, 1, b"", 1, 0), (640, 0, 127, b"", 1, 0),
        # inside (AC) x 100: one unit deleted / inserted anywhere
        (1100, 0, 2, b"", 1, 0), (1151, 0, 2, b"", 0, 1), (1198, 0, 2, b"", 1, 0), (1100, 1, 2, b"AC", 1, 0), (1101, 1, 2, b"CA", 0, 1),
        (1200, 1, 2, b"AC", 1, 0), (1100, 0, 4, b"", 2, 0), (1100, 1, 3, b"ACA", 1, 0),
        # next to a separator: stops behind it; at a record's first letter; at row 0
        (2004, 0, 1, b"", 1, 0), (2003, 0, 2, b"", 0, 1), (2005, 1, 1, b"T", 1, 0), (2001, 1, 3, b"GGT", 1, 0), (3501, 0, 5, b"", 0, 1),
        (0, 0, 1, b"", 1, 0), (0, 1, 2, b"CC", 1, 1), (4999, 0, 1, b"", 1, 0), (4999, 1, 1, bytes([T[4998] & 0xDF]), 1, 0),
        (4206, 1, 4, b"ACGT", 2, 0), (4208, 0, 4, b"", 0, 3),
        # the same key twice in one call
        (3000, 1, 2, b"GA", 10, 20), (1100, 0, 2, b"", 7, 7),
    ]
    order = rng.permutation(len(ev))
    return [ev[i] for i in order]


def test_planted_events_ranges_and_capacity(eng):
    import torch
    from slamem_amd import capi
    text = planted_text()
    n = len(text)
    idx = eng.Index.build(text)
    p = eng.Pileup(idx, events=True, event_slots=64)
    ev = plants(text)
    spec = es.Table(text)
    for e in ev:
        spec.observe(*e)
    want = spec.events()
    assert 25 <= len(want) <= 64 and spec.skipped == [0, 0, 0] and len(want) < len(ev)
    # (the plants do what the docstring says)
    keys = {w[:4] for w in want}
    assert {(500, 0, 3, b""), (500, 1, 2, b"AA"), (500, 0, 1, b""), (500, 0, 127, b""), (1000, 0, 2, b""), (1000, 1, 2, b"AC"),
            (2001, 0, 1, b""), (2001, 0, 2, b""), (2001, 1, 1, b"T"), (3501, 0, 5, b""), (0, 0, 1, b"")} <= keys
    p.add_events(es.to_records(ev))
    got, skipped = got_events(p)
    assert got == want and skipped == [0, 0, 0]
    for kw in (dict(first=3000), dict(first=3001), dict(first=3000, count=1), dict(first=2900, count=100), dict(first=2900, count=101),
               dict(first=1200, count=800), dict(first=n, count=0), dict(first=0, count=0), dict(first=0, count=1), dict(first=4999, count=1),
               dict(min_count=4), dict(min_count=5), dict(min_count=34), dict(min_count=35), dict(min_count=2, first=500, count=501)):
        assert got_events(p, **kw)[0] == spec.events(kw.get("first", 0), kw.get("count"), kw.get("min_count", 1)), kw
    assert spec.events(first=1200, count=800) == [] and len(spec.events(min_count=34)) == 1 and spec.events(min_count=35) == []
    # the read-out left the table alone; a canonical event added again stays where it is
    assert got_events(p)[0] == want
    # a capacity that is too small: the need, a correct prefix, nothing behind it
    L = capi.lib()
    dev = idx.device
    cap = 5
    buf = torch.full(((cap + 4) * 32,), 0x5A, dtype=torch.uint8, device=dev)
    total, sk = C.c_uint64(), (C.c_uint64 * 3)()
    rc = L.slamem_pileup_events_device(p._h, 0, n, 1, cap, buf.data_ptr(), sk, C.byref(total), None)
    torch.cuda.synchronize()
    assert rc == capi.SLAMEM_ERR_CAPACITY and total.value == len(want) and b"selected" in L.slamem_last_error_message()
    assert bool((buf[cap * 32:] == 0x5A).all())
    assert es.from_records(buf[:cap * 32].cpu().numpy().view(eng.EVENT_DTYPE)) == want[:cap]
    rc = L.slamem_pileup_events_device(p._h, 0, n, 1, 0, None, sk, C.byref(total), None)
    assert rc == capi.SLAMEM_ERR_CAPACITY and total.value == len(want)
    host = np.zeros(len(want) + 2, dtype=eng.EVENT_DTYPE)
    rc = L.slamem_pileup_events_host(p._h, 0, n, 1, 3, host.ctypes.data, sk, C.byref(total))
    assert rc == capi.SLAMEM_ERR_CAPACITY and total.value == len(want) and es.from_records(host[:3]) == want[:3] and not host[3:]["fwd"].any()
    rc = L.slamem_pileup_events_host(p._h, 0, n, 1, len(host), host.ctypes.data, sk, C.byref(total))
    assert rc == capi.SLAMEM_OK and es.from_records(host[:total.value]) == want
    assert got_events(p, capacity=3)[0] == want
    # merged into a second accumulator through the host call, the events stay as they are; reset clears them
    q = eng.Pileup(idx, events=True, event_slots=128)
    assert L.slamem_pileup_add_events_host(q._h, host.ctypes.data, len(want)) == capi.SLAMEM_OK
    assert got_events(q)[0] == want
    for e in (eng.event_letters(x) for x in p.events()[0]):
        assert isinstance(e, bytes)
    assert [eng.event_letters(x) for x in p.events()[0]] == [w[3] for w in want]
    p.reset()
    assert got_events(p) == ([], [0, 0, 0])
    # refusals
    for bad in (dict(first=n + 1, count=0), dict(first=n - 1, count=2), dict(min_count=0)):
        with pytest.raises(capi.SlamemError) as err:
            p.events(**bad)
        assert err.value.code == capi.SLAMEM_ERR_ARG
    plain = eng.Pileup(idx)
    for call in (lambda: plain.events(), lambda: plain.add_events(es.to_records(ev[:1]))):
        with pytest.raises(capi.SlamemError) as err:
            call()
        assert err.value.code == capi.SLAMEM_ERR_ARG and "not enabled" in str(err.value)
    assert L.slamem_pileup_enable_events(p._h, 64) == capi.SLAMEM_ERR_ARG and b"already" in L.slamem_last_error_message()
    for slots in (63, 32, 100, 2 ** 32):
        assert L.slamem_pileup_enable_events(plain._h, slots) == capi.SLAMEM_ERR_ARG
    assert L.slamem_pileup_enable_events(plain._h, 0) == capi.SLAMEM_OK  # the default
    assert got_events(plain) == ([], [0, 0, 0])
    for x in (p, q, plain):
        x.close()
    idx.close()


# ---- contention ----------------------------------------------------------------------------------------------------------------

def test_contention_on_one_key_and_on_the_alleles_of_one_position(eng):
    import torch
    text = planted_text()
    idx = eng.Index.build(text)
    p = eng.Pileup(idx, events=True, event_slots=256)
    one = np.zeros(100_000, dtype=eng.EVENT_DTYPE)
    one["pos"], one["kind"], one["len"], one["fwd"] = 700, 0, 3, 1  # (un-normalised: every lane walks the run first)
    p.add_events(one)
    assert got_events(p) == ([(500, 0, 3, b"", 100_000, 0)], [0, 0, 0])
    p.reset()
    # 64 alleles at one position (all share key0: a probe sequence of 64 slots), 1,000 observations each, shuffled
    rng = np.random.default_rng(31)
    alleles = [bytes([a, b, c]) for a in b"ACGT" for b in b"ACGT" for c in b"ACGT"]
    rows = es.to_records([(3501, 1, 3, S, 1, 0) for S in alleles] * 500 + [(3501, 1, 3, S, 0, 1) for S in alleles] * 500)
    rows = rows[rng.permutation(len(rows))]
    p.add_events(rows)
    want = [(3501, 1, 3, S, 500, 500) for S in sorted(alleles)]
    assert got_events(p) == (want, [0, 0, 0])
    # the same, split over two host threads and two HIP streams into one accumulator
    p.reset()
    dev = idx.device
    errs = []

    def worker(part):
        try:
            with torch.cuda.stream(torch.cuda.Stream(dev)):
                for piece in np.array_split(part, 4):
                    p.add_events(piece)
        except Exception as e:  # noqa: BLE001
            errs.append(e)
    th = [threading.Thread(target=worker, args=(rows[k::2],)) for k in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs
    torch.cuda.synchronize()
    assert got_events(p) == (want, [0, 0, 0])
    p.close()
    idx.close()


def test_full_table_counts_what_it_could_not_store(eng):
    text = planted_text()
    idx = eng.Index.build(text)
    p = eng.Pileup(idx, events=True, event_slots=64)
    rng = np.random.default_rng(37)
    ev = [(2100 + 5 * k, 1, 1, bytes([b"ACGT"[(b"ACGT".index(bytes([text[2100 + 5 * k - 1] & 0xDF])) + 1) % 4]]), int(rng.integers(1, 9)),
           int(rng.integers(0, 9))) for k in range(200)]
    spec = es.Table(text)
    for e in ev:
        spec.observe(*e)
    assert len(spec.keys) == 200 and all(e[:4] in spec.keys for e in ev)  # (200 distinct canonical keys)
    p.add_events(es.to_records(ev))
    p.add_events(es.to_records(ev))
    got, skipped = got_events(p)
    assert 0 < len(got) <= 64 and skipped[0] == 0 and skipped[2] == 0
    for g in got:  # every key that got in carries its exact counts
        c = spec.keys[g[:4]]
        assert (g[4], g[5]) == (2 * c[0], 2 * c[1])
    assert sum(g[4] + g[5] for g in got) + skipped[1] == 2 * sum(e[4] + e[5] for e in ev)
    p.close()
    idx.close()


# ---- crafted batches: the skipped counters, the lane kernel and the wave kernel ------------------------------------------------

def craft(eng, idx, p, reads, results, min_mapq=0):
    """Adds a batch written out by hand: results are read_map tuples (strand, mapq, s1, s2, segments)."""
    import torch
    dev = idx.device
    q = np.concatenate([np.frombuffer(r, dtype=np.uint8) for r in reads] + [np.zeros(8, dtype=np.uint8)])
    off = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.uint64)
    segs, roff, ops, ooff, recs = [], [0], [], [0], []
    code = {"=": 7, "X": 8, "I": 1, "D": 2}
    for strand, mapq, s1, s2, segl in results:
        for (rp, qp, rlen, qlen, ed, rl) in segl:
            segs.append((rp, qp, rlen, qlen, ed))
            ops += [(k << 4) | code[c] for c, k in rl]
            ooff.append(len(ops))
        roff.append(len(segs))
        recs.append(np.array([(s1, s2, strand, mapq, 0, 0)], dtype=np.dtype([("s1", "<u4"), ("s2", "<u4"), ("strand", "u1"), ("mapq", "u1"),
                                                                                    ("r0", "u1"), ("r1", "u1")])))
    dv = lambda a, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dt)).view(np.uint8).reshape(-1).copy()).to(dev)  # noqa: E731
    p._add_device(dv(q, np.uint8), dv(off, np.uint64), len(reads), dv(np.array(segs, dtype=np.uint32).reshape(-1, 5), np.uint32),
                  dv(roff, np.uint64), dv(ops + [0], np.uint32), dv(ooff, np.uint64), dv(np.concatenate(recs).view(np.uint8), np.uint8), min_mapq)
    return q[:-8], off


def test_skips_go_to_their_counters_and_nowhere_else(eng):
    text = planted_text()
    n = len(text)
    idx = eng.Index.build(text)
    p = eng.Pileup(idx, events=True, event_slots=64)
    # through add_events: an insertion of 32 letters, at row n, letters beyond the length, a deletion over a separator / of 128 rows
    bad = es.to_records([(3000, 1, 31, b"C" * 31, 2, 1), (n, 1, 1, b"C", 1, 1), (3000, 1, 2, b"CC", 1, 0), (1999, 0, 3, b"", 0, 4),
                         (2600, 0, 127, b"", 1, 0), (n - 1, 0, 2, b"", 1, 0), (3000, 0, 1, b"", 0, 0)])
    bad[0]["len"] = 32
    bad[2]["letters"] = 1 << 4
    bad[4]["len"] = 128
    p.add_events(bad)
    assert got_events(p) == ([], [3, 0, 2 + 1 + 4 + 1 + 1])
    p.reset()
    # through an add: a read whose insertion holds an N, one of 33 letters, an insertion at row n, a deletion that runs past n --
    # and two valid ones; strand 2 is scanned as its reverse complement; a read below the quality does not count
    r0 = b"ACGTACNTAC"
    r1 = b"ACGT" + b"G" * 33 + b"ACGT"
    r2 = bytes(text[3000:3004]) + b"GA" + bytes(text[3004:3008])
    fw = bytes(text[3100:3105]) + bytes(text[3108:3112])  # rows 3105..3107 deleted
    r3 = bytes(es.ext_spec.revcomp(np.frombuffer(fw, dtype=np.uint8)))
    r4 = b"ACGTAC"
    results = [
        (1, 60, 10, 0, [(100, 0, 7, 10, 3, [("=", 4), ("I", 3), ("=", 3)])]),
        (1, 60, 10, 0, [(200, 0, 8, 41, 33, [("=", 4), ("I", 33), ("=", 4)])]),
        (1, 60, 10, 0, [(3000, 0, 8, 10, 2, [("=", 4), ("I", 2), ("=", 4)])]),
        (2, 30, 10, 0, [(3100, 0, 12, 9, 3, [("=", 5), ("D", 3), ("=", 4)])]),
        (1, 60, 10, 0, [(n - 4, 0, 4, 6, 2, [("=", 4), ("I", 2)]), (n - 2, 0, 5, 0, 5, [("D", 5)])]),
        (1, 10, 10, 0, [(3000, 0, 8, 10, 2, [("=", 4), ("I", 2), ("=", 4)])]),
        (0, 0, 0, 0, []),
    ]
    reads = [r0, r1, r2, r3, r4, r2, b"ACGT"]
    q, off = craft(eng, idx, p, reads, results, min_mapq=20)
    spec = es.Table(text).add_batch(results, q, off, 20)
    assert spec.skipped == [1, 0, 3] and len(spec.keys) == 2
    assert got_events(p) == (spec.events(), spec.skipped)
    assert [g[4:] for g in got_events(p)[0]] in ([(1, 0), (0, 1)], [(0, 1), (1, 0)])
    p.close()
    idx.close()


def test_lane_and_wave_kernels_on_a_crafted_batch(eng):
    """Segments of 3, 32, 33 and 130 operations with an indel every few letters, on both strands: the lane kernel takes the first
    two, the wave kernel the others (two rounds of 64 operations and a rest)."""
    rng = np.random.default_rng(41)
    text = planted_text()
    idx = eng.Index.build(text)
    reads, results = [], []
    for k, nops in enumerate((3, 32, 33, 130, 64, 65)):
        rl = []
        for j in range(nops):
            rl.append(("=", 2) if j % 2 == 0 else (("I", 1 + j % 3) if j % 4 == 1 else ("D", 1 + j % 2)))
        qlen = sum(c for o, c in rl if o in "=I")
        rlen = sum(c for o, c in rl if o in "=D")
        start = 2100 + 400 * k
        strand = 1 + k % 2
        reads.append(bytes(rng.choice(ACGT, size=qlen)))
        results.append((strand, 60, 10, 0, [(start, 0, rlen, qlen, 0, rl)]))
    p = eng.Pileup(idx, events=True, event_slots=1024)
    q, off = craft(eng, idx, p, reads, results)
    spec = es.Table(text).add_batch(results, q, off)
    assert len(spec.keys) > 60 and spec.skipped == [0, 0, 0]
    assert got_events(p) == (spec.events(), [0, 0, 0])
    p.close()
    idx.close()


# ---- real mappings -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["indel_reads", "multi_record"])
def test_real_mappings_any_order_the_stream_and_a_merge(eng, case):
    if case == "indel_reads":
        ref, q, off = indel_reads(21)
        min_len = 14
    else:
        ref, q, off = multi_record_batch()
        min_len = 20
    idx = eng.Index.build(ref)
    res = spec_results(idx, ref, q, off, min_len, True)
    want = es.events(res, q, off, ref)
    p = eng.Pileup(idx, events=True)
    p.add(q, off, min_len, True)
    assert got_events(p) == want
    if case == "indel_reads":
        assert len(want[0]) > 50 and any(e[1] == 0 for e in want[0]) and any(e[1] == 1 for e in want[0])
        assert any(e[4] for e in want[0]) and any(e[5] for e in want[0])
    # with events enabled the pileup itself is what it is without them
    plain = eng.Pileup(idx)
    plain.add(q, off, min_len, True)
    table = plain.counts()
    assert np.array_equal(p.counts(), table)
    for g, w in zip(p.sites(1, 0), plain.sites(1, 0)):
        assert np.array_equal(g, w)
    plain.close()
    # a minimum quality
    p.reset()
    p.add(q, off, min_len, True, min_mapq=30)
    assert got_events(p) == es.events(res, q, off, ref, 30)
    # the halves in the other order
    (qa, oa), (qb, ob) = halves(q, off)
    p.reset()
    p.add(qb, ob, min_len, True)
    p.add(qa, oa, min_len, True)
    assert got_events(p) == want
    # a stream of match type 8 feeds the accumulator
    p.reset()
    run_stream(eng, idx, p, q, windows(off, (len(off) - 1 + 2) // 3), 2, min_len)
    assert got_events(p) == want and np.array_equal(p.counts(), table)
    # two accumulators, a half each, merged
    a, b = eng.Pileup(idx, events=True), eng.Pileup(idx, events=True, event_slots=4096)
    a.add(qa, oa, min_len, True)
    b.add(qb, ob, min_len, True)
    a.add_events(b.events()[0])
    assert got_events(a) == want
    # rows_at: what counts() has there -- tile borders, the ends, a separator or an uncovered row, rows under the reads
    n = len(ref)
    pos = [0, 2047, 2048, 4095, 4096, n - 1, 3000, 8001] + [int(e[0]) for e in want[0][:50]] + [max(int(e[0]) - 1, 0) for e in want[0][:50]]
    assert np.array_equal(p.rows_at(pos), table[pos])
    assert np.array_equal(p.rows_at(pos + [n, n + 5])[-2:], np.zeros((2, 6), dtype=np.uint32))
    assert p.rows_at([]).shape == (0, 6)
    from slamem_amd import capi
    L = capi.lib()
    hp, out = np.array(pos, dtype=np.uint64), np.zeros((len(pos), 6), dtype=np.uint32)
    assert L.slamem_pileup_rows_at_host(p._h, hp.ctypes.data, len(hp), out.ctypes.data) == capi.SLAMEM_OK and np.array_equal(out, table[pos])
    hp[3] = n
    assert L.slamem_pileup_rows_at_host(p._h, hp.ctypes.data, len(hp), out.ctypes.data) == capi.SLAMEM_ERR_ARG
    for x in (a, b, p):
        x.close()
    idx.close()


def test_planted_deletion_in_a_homopolymer_is_one_event(eng):
    """A known answer, judged without the spec: a random reference with a run of eight A, a sample that lacks three of them, 20
    error-free reads of 150 letters across the place, alternating strands.  Wherever the aligner puts the gap inside the run, the
    table holds one event: a deletion of 3 at the run's first letter, seen 20 times.
    test_events_host.test_planted_deletion_answer_holds_on_the_definition confirms the answer on the CPU."""
    ref, run_start, q, off = planted_deletion()
    idx = eng.Index.build(ref)
    p = eng.Pileup(idx, events=True)
    recs = p.add(q, off, 20, True)
    assert np.array_equal(recs["strand"], 1 + np.arange(len(off) - 1) % 2)
    arr, skipped = p.events()
    print("events", arr.tolist(), skipped)
    assert len(arr) == 1 and skipped == [0, 0, 0]
    e = arr[0]
    assert (int(e["pos"]), int(e["kind"]), int(e["len"]), int(e["letters"])) == (run_start, 0, 3, 0)
    assert int(e["fwd"]) + int(e["rev"]) == 20 and int(e["fwd"]) == 10
    p.close()
    idx.close()


# ---- the executable ------------------------------------------------------------------------------------------------------------

def test_cli_file_is_the_spec_of_the_engines_tables(eng, tmp_path):
    """slaMEM-hip -b -l 14 -vcf -mdep 1 -mpct 0 ref.fa reads.fa on a reference of two records: byte for byte the file events_spec
    formats from the engine's pileup and events; the same with two logical GPUs (the tables and the events merged on GPU 0) and
    with a small event table given by -evs; at the defaults another file."""
    import hostlib
    ref, q, off = indel_reads(21)
    ref = ref.copy()
    ref[20000] = ord("N")  # (no read lies across it)
    recs = [ref[:20000], ref[20001:]]
    ref_fa, q_fa = str(tmp_path / "ref.fa"), str(tmp_path / "reads.fa")
    write_fasta(ref_fa, [(b"one first", recs[0]), (b"two\tsecond", recs[1])])
    write_fasta(q_fa, [(b"read%d x" % k, q[int(off[k]):int(off[k + 1])]) for k in range(len(off) - 1)])
    loaded = hostlib.Loaded(ref_fa, 1)
    assert loaded.chars == bytes(ref)
    idx = eng.Index.build(ref)
    p = eng.Pileup(idx, events=True)
    p.add(q, off, 14, True)
    table = p.counts().astype(np.int64)
    ev = es.from_records(p.events()[0])
    p.close()
    idx.close()
    want = es.vcf_file(table, ev, loaded, 1, 0)
    dflt = es.vcf_file(table, ev, loaded)
    head = es.vcf_header(loaded)
    assert want.startswith(head) and want.count(b";SF=") > 50 and want.count(b"\n") > want.count(b";SF=") + 50 and want != dflt
    assert b"\none\t" in want and b"\ntwo\t" in want
    base = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for name, env, extra in (("one", base, []), ("two", dict(base, SLAMEM_LOGICAL_GPUS="2", SLAMEM_BATCH_MB="1"), []),
                             ("evs", base, ["-evs", "4096"])):
        out = str(tmp_path / (name + ".vcf"))
        r = subprocess.run([EXE, "-b", "-l", "14", "-vcf", "-mdep", "1", "-mpct", "0", "-o", out] + extra + [ref_fa, q_fa],
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=300)
        assert r.returncode == 0, (r.stdout + r.stderr).decode(errors="replace")[-3000:]
        assert open(out, "rb").read() == want
        assert b"Saving variant calls" in r.stdout and b"; minimum depth = 1 ; minimum share = 0 %\n" in r.stdout
        assert b"WARNING" not in r.stderr
    r = subprocess.run([EXE, "-vcf", "-b", "-l", "14", ref_fa, q_fa], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=base, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr).decode(errors="replace")[-3000:]
    assert open(str(tmp_path / "ref-mems.txt"), "rb").read() == dflt
    # a table that is too small says so on stderr, with the hint
    out = str(tmp_path / "small.vcf")
    r = subprocess.run([EXE, "-b", "-l", "14", "-vcf", "-evs", "64", "-o", out, ref_fa, q_fa], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       env=base, timeout=300)
    assert r.returncode == 0 and open(out, "rb").read().startswith(head)
    assert (b"WARNING" in r.stderr) == (len(ev) > 64) and (b"-evs" in r.stderr) == (len(ev) > 64)


@pytest.mark.parametrize("args,message", [
    (["-vcf", "-sites"], b"Option -vcf excludes -mam, -mum, -smem, -chain, -ext, -aln, -paf, -pile and -sites"),
    (["-pile", "-evs", "64"], b"Option -evs needs -vcf"),
    (["-vcf", "-evs", "96"], b"Option -evs needs a power of two of at least 64"),
])
def test_cli_refusals(args, message, tmp_path):
    ref_fa, q_fa = str(tmp_path / "ref.fa"), str(tmp_path / "reads.fa")
    write_fasta(ref_fa, [(b"r", b"ACGT" * 30)])
    write_fasta(q_fa, [(b"q", b"ACGT" * 10)])
    r = subprocess.run([EXE] + args + [ref_fa, q_fa], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60)
    assert r.returncode == 255 and message in r.stdout and b"Building index" not in r.stdout
