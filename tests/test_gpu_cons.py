"""-cons on the MI355X (slamem_pileup_consensus_*, engine.Pileup.consensus, the executable): every output is tests/cons_spec.py
applied to the same table and events, compared for exact equality of bytes, offs and statistics -- planted tables in which every
rule and tie occurs, the edges of the read-out's tiles of 2,048 rows, the capacity rule, the refusals -- and, without the spec, a
known answer: reads of a sample with 20 SNVs, a deletion and an insertion give the sample back."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cons_spec as cs
import events_spec as es
import ext_spec
from test_gpu_events import planted_text, plants
from test_gpu_sites import halves, write_fasta

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "slamem_amd", "host", "slaMEM-hip")
TILE = 2048


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test without a GPU")
    from slamem_amd import engine
    return engine


def check(p, text, table, E, md, first=0, count=None, bounds=()):
    got, offs, stats = p.consensus(md, first, count, bounds=list(bounds) if len(bounds) else None)
    want, woffs, wstats = cs.consensus(text, table, E, md, first, count, bounds)
    assert got.dtype == np.uint8 and offs.dtype == np.uint64
    assert bytes(got) == want, (md, first, count)
    assert [int(v) for v in offs] == woffs and stats == wstats, (md, first, count)
    return want


def own_column(text):
    code = np.full(len(text), 4, dtype=np.int64)
    for k, c in enumerate(b"ACGT"):
        code[(np.asarray(text) & 0xDF) == c] = k
    return code


# ---- planted -------------------------------------------------------------------------------------------------------------------

def planted_table(text, rng):
    """Rows of seven kinds, so that every rule and every tie occurs."""
    n = len(text)
    own = own_column(text)
    t = np.zeros((n, 6), dtype=np.uint32)
    kind = rng.integers(0, 7, size=n)
    for p in range(n):
        o, k = int(own[p]) % 4, int(kind[p])
        other = (o + 1 + int(rng.integers(0, 3))) % 4
        if k == 1:    # shallow
            t[p][o] = rng.integers(1, 4)
        elif k == 2:  # deep, but no letter seen
            t[p][4] = rng.integers(4, 9)
        elif k == 3:  # the text's letter wins
            t[p][o], t[p][other] = rng.integers(10, 40), rng.integers(0, 10)
        elif k == 4:  # another letter wins
            t[p][other], t[p][o], t[p][4] = rng.integers(10, 40), rng.integers(0, 10), rng.integers(0, 3)
        elif k == 5:  # a tie with the text's letter
            t[p][o] = t[p][other] = rng.integers(2, 9)
        elif k == 6:  # a tie without it
            a, b = [x for x in range(4) if x != o][:2] if rng.integers(0, 2) else [x for x in range(4) if x != o][1:]
            t[p][a] = t[p][b] = rng.integers(2, 9)
            t[p][o] = rng.integers(0, 2)
        t[p][5] = rng.integers(0, 3)
    return t


def planted_case():
    rng = np.random.default_rng(43)
    text = planted_text()
    n = len(text)
    T = bytes(text)
    raw = [(p, kind, k, S, 3 * f, 3 * r) for (p, kind, k, S, f, r) in plants(text)]

    def unlike(p):  # a letter that the row in front of p does not hold: an insertion that ends with it stays at p
        return bytes([b"ACGT"[(b"ACGT".index(bytes([T[p - 1] & 0xDF])) + 1) % 4]])
    raw += [(4500, 1, 2, b"G" + unlike(4500), 3, 3), (4500, 1, 2, b"C" + unlike(4500), 6, 0), (4500, 1, 1, unlike(4500), 2, 2),  # equal obs
            (2000, 1, 2, b"T" + unlike(2000), 4, 4), (1998, 0, 2, b"", 5, 0),  # in front of a separator
            (3501, 1, 3, b"ACG", 2, 3), (3499, 0, 1, b"", 4, 0)]
    spec = es.Table(text)
    for e in raw:
        spec.observe(*e)
    E = spec.events()
    assert spec.skipped == [0, 0, 0]
    t = planted_table(text, rng)
    own = own_column(text)
    special = (0, 1998, 2000, 3501, 4500, 4999)  # the ends, the separators' neighbours, the trio at 4500
    for i, e in enumerate(E):  # every third event: an anchor row of depth 40, which few events reach half of
        a = cs.anchor(T, e[0])
        if i % 3 == 1 and own[a] < 4:
            t[a] = 0
            t[a][own[a]] = 40
    for i, e in enumerate(E):  # every third event, the longest ones and the special ones: an anchor row of depth 4
        a = cs.anchor(T, e[0])
        if (i % 3 == 0 or e[2] in (31, 127) or e[0] in special) and own[a] < 4:
            t[a] = 0
            t[a][own[a]] = 4
    return text, t, raw, E


def test_planted_tables_every_rule_with_and_without_events(eng):
    text, t, raw, E = planted_case()
    T, n = bytes(text), len(text)
    # the plants do what the docstring says
    rows = {(cs.row(T, t, p, 4)[0], cs.row(T, t, p, 4)[2]) for p in range(n)}
    assert rows == {("N", ""), ("uncalled", ""), ("called", ""), ("called", "own"), ("called", "first")}
    assert any(cs.row(T, t, p, 4)[0] == "uncalled" and cs.depth(t, p) >= 4 for p in range(n))
    app = [cs.applied(T, t, e, 4) for e in E]
    for kind in (0, 1):
        assert any(a and e[1] == kind for a, e in zip(app, E)) and any(not a and e[1] == kind for a, e in zip(app, E))
    assert any(a and e[1] == 1 and e[2] == 31 for a, e in zip(app, E)) and any(a and e[1] == 0 and e[2] == 127 for a, e in zip(app, E))
    at = [e for a, e in zip(app, E) if a and e[0] == 4500 and e[1] == 1]
    assert len(at) == 3 and [e[4] + e[5] for e in at] == [4, 6, 6]  # (the second wins: the first of the tied)
    pos = {e[0] for a, e in zip(app, E) if a}
    assert {0, n - 1, 2000, 3501} <= pos and any(e[0] < 2000 <= e[0] + e[2] - 1 or e[0] + e[2] == 2000 for a, e in zip(app, E) if a and e[1] == 0)
    em = cs.emissions(T, t, E, 4)
    assert any(S and rule == "deleted" for S, rule, _ in em) and {r for _, r, _ in em} == set(cs.RULES)

    idx = eng.Index.build(text)
    p = eng.Pileup(idx, events=True, event_slots=256)
    p.add_counts(t)
    p.add_events(es.to_records(raw))
    assert es.from_records(p.events()[0]) == E and np.array_equal(p.counts(), t)
    bounds = [0, 1, 2000, 2001, 2047, 2048, 3500, 3501, 4999, n]
    whole = {}
    for md in (1, 4, 2 ** 31 - 1):
        whole[md] = check(p, T, t, E, md, bounds=bounds)
    assert whole[1] != whole[4] and whole[2 ** 31 - 1] == bytes(c if c == ord("N") else c | 0x20 for c in T).replace(b"n", b"N")
    # ranges are slices: one inside a deletion of 127 rows, one that starts behind an event's anchor, the separators
    d127 = next(e for a, e in zip(app, E) if a and e[1] == 0 and e[2] == 127)
    for first, count in ((d127[0] + 5, 100), (d127[0] + 126, 3), (2000, 2), (3501, 1499), (4500, 1), (0, 1), (n - 1, 1), (n, 0), (0, 0),
                         (2040, 20)):
        check(p, T, t, E, 4, first, count, bounds=[first, first + count // 2, first + count])
    # the read-outs of the table and of the events are what they were
    assert es.from_records(p.events()[0]) == E and np.array_equal(p.counts(), t)
    # without events the table alone decides
    plain = eng.Pileup(idx)
    plain.add_counts(t)
    for md in (1, 4, 2 ** 31 - 1):
        assert check(plain, T, t, [], md, bounds=bounds) != whole[1]
    check(plain, T, t, [], 4, 2047, 2)
    plain.close()
    p.close()
    idx.close()


# ---- tile edges ----------------------------------------------------------------------------------------------------------------

def unlike_before(T, p):
    return bytes([b"ACGT"[(b"ACGT".index(bytes([T[p - 1] & 0xDF])) + 1) % 4]])


@pytest.mark.parametrize("n", [2047, 2048, 2049, 4097])
def test_tile_edges_ranges_and_bounds(eng, n):
    rng = np.random.default_rng(n)
    text = rng.choice(ACGT, size=n)
    text[100:110] |= 0x20
    if n > 2047:  # the deletion from 2046 stays there
        dl = min(4, n - 2046)
        text[2045] = ACGT[(int(np.where(ACGT == text[2046 + dl - 1])[0][0]) + 1) % 4]
    T = bytes(text)
    own = own_column(text)
    t = np.zeros((n, 6), dtype=np.uint32)
    t[np.arange(n), own] = 6
    snv = rng.choice(n, size=60, replace=False)
    t[snv, (own[snv] + 1) % 4] = 9
    t[rng.choice(n, size=40, replace=False)] = 0
    for a in (0, 2045, 2046, 2047, n - 2):  # the anchors of the events below
        if a < n:
            t[a] = 0
            t[a][own[a]] = 6
    raw = [(1, 1, 1, unlike_before(T, 1), 4, 0), (n - 1, 0, 1, b"", 0, 4), (2046, 1, 2, b"A" + unlike_before(T, 2046), 2, 2)]
    if n > 2047:
        raw += [(2046, 0, dl, b"", 4, 0), (2047, 1, 2, b"G" + unlike_before(T, 2047), 4, 0)]
    if n > 2048:
        raw += [(2048, 1, 3, b"CA" + unlike_before(T, 2048), 3, 1)]
    spec = es.Table(text)
    for e in raw:
        spec.observe(*e)
    E = spec.events()
    keys = {e[:3] for e in E if cs.applied(T, t, e, 4)}
    assert (1, 1, 1) in keys and (2046, 1, 2) in keys
    assert n <= 2047 or ({(2046, 0, dl), (2047, 1, 2)} <= keys)
    assert n <= 2048 or (2048, 1, 3) in keys
    idx = eng.Index.build(text)
    p = eng.Pileup(idx, events=True, event_slots=64)
    p.add_counts(t)
    p.add_events(es.to_records(raw))
    marks = [0, 1, 2046, 2047, 2048, 2049, 4095, 4096, n]
    check(p, T, t, E, 4, bounds=[b for b in marks if b <= n])
    done = 0
    for first in (1, 2047, 2048):
        for count in (0, 1, 2049):
            if first + count > n:
                continue
            check(p, T, t, E, 4, first, count, bounds=[b for b in [first] + marks + [first + count] if first <= b <= first + count])
            done += 1
    assert done >= (3 if n == 2047 else 4)
    if n > 2048:  # (the anchor of the insertion at 2048 is row 2047, in front of the range)
        assert bytes(p.consensus(4, 2048, 1)[0][:3]) == next(e[3] for e in E if e[:3] == (2048, 1, 3))
    p.close()
    idx.close()


def test_a_tile_that_emits_nothing_and_a_tile_of_insertions(eng):
    """4,097 rows: every row of tile 0 carries an insertion of one letter, and chained deletions of 127 rows take all of tile 1."""
    n = 4097
    rng = np.random.default_rng(47)
    text = rng.choice(ACGT, size=n)
    starts = list(range(TILE, 2 * TILE, 127))
    for i, s in enumerate(starts + [2 * TILE]):  # the rows in front of the deletions and the last row: a deletion stays where it is
        text[s - 1] = ACGT[i % 2]
    T = bytes(text)
    own = own_column(text)
    t = np.zeros((n, 6), dtype=np.uint32)
    t[np.arange(n), own] = 4
    raw = [(s, 0, min(127, 2 * TILE - s), b"", 2, 1) for s in starts]
    raw += [(p, 1, 1, unlike_before(T, p) if p else b"G", 1, 2) for p in range(TILE)]
    spec = es.Table(text)
    for e in raw:
        spec.observe(*e)
    E = spec.events()
    assert len(E) == len(raw) and all(cs.applied(T, t, e, 4) for e in E)
    em = cs.emissions(T, t, E, 4)
    assert all(S and rule == "called" for S, rule, _ in em[:TILE]) and all(not S and rule == "deleted" for S, rule, _ in em[TILE:2 * TILE])
    assert em[2 * TILE][1] == "called"
    idx = eng.Index.build(text)
    p = eng.Pileup(idx, events=True, event_slots=8192)
    p.add_counts(t)
    p.add_events(es.to_records(raw))
    want = check(p, T, t, E, 4, bounds=[0, 1, 2047, 2048, 2049, 4095, 4096, 4097])
    assert len(want) == 2 * TILE + 1
    assert p.consensus(4, 2048, 2048)[0].size == 0 and p.consensus(4, 2048, 2048)[2] == [0, 0, 2048, 0, 0]
    check(p, T, t, E, 4, 2047, 2050, bounds=[2047, 2048, 4096, 4097])
    check(p, T, t, E, 4, 1, 2049, bounds=[1, 2050])
    p.close()
    idx.close()


# ---- the C ABI: capacity, refusals, host buffers -------------------------------------------------------------------------------

def test_capacity_refusals_and_the_host_variant(eng):
    import torch
    from slamem_amd import capi
    text, t, raw, E = planted_case()
    T, n = bytes(text), len(text)
    idx = eng.Index.build(text)
    p = eng.Pileup(idx, events=True, event_slots=256)
    p.add_counts(t)
    p.add_events(es.to_records(raw))
    want, _, wstats = cs.consensus(T, t, E, 4)
    need = len(want)
    L = capi.lib()
    dev = idx.device
    cap = need - 1
    buf = torch.full((need + 64,), 0x5A, dtype=torch.uint8, device=dev)
    total, stats = C.c_uint64(), (C.c_uint64 * 5)()
    rc = L.slamem_pileup_consensus_device(p._h, 0, n, 4, cap, buf.data_ptr(), None, 0, None, stats, C.byref(total), None)
    torch.cuda.synchronize()
    assert rc == capi.SLAMEM_ERR_CAPACITY and total.value == need and list(stats) == wstats
    assert bool((buf[cap:] == 0x5A).all()) and bytes(buf[:cap].cpu().numpy()) == want[:cap]
    for small in (1, 63, 2049):
        buf.fill_(0x5A)
        rc = L.slamem_pileup_consensus_device(p._h, 0, n, 4, small, buf.data_ptr(), None, 0, None, stats, C.byref(total), None)
        torch.cuda.synchronize()
        assert rc == capi.SLAMEM_ERR_CAPACITY and total.value == need
        assert bool((buf[small:] == 0x5A).all()) and bytes(buf[:small].cpu().numpy()) == want[:small]
    rc = L.slamem_pileup_consensus_device(p._h, 0, n, 4, 0, None, None, 0, None, stats, C.byref(total), None)
    assert rc == capi.SLAMEM_ERR_CAPACITY and total.value == need and list(stats) == wstats
    got = p.consensus(4, capacity=3)  # (the engine asks once more with the need)
    assert bytes(got[0]) == want and got[2] == wstats
    # bounds on the device: one outside the range is answered with all ones
    first, count = 2000, 1000
    b = np.array([2000, 2500, 3000, 1999, 3001, 2 ** 40], dtype=np.uint64)
    bd = torch.from_numpy(b.view(np.int64)).to(dev)
    od = torch.zeros(len(b), dtype=torch.int64, device=dev)
    part, poffs, _ = cs.consensus(T, t, E, 4, first, count, [2000, 2500, 3000])
    rc = L.slamem_pileup_consensus_device(p._h, first, count, 4, 0, None, bd.data_ptr(), len(b), od.data_ptr(), stats, C.byref(total), None)
    torch.cuda.synchronize()
    assert rc == capi.SLAMEM_ERR_CAPACITY and total.value == len(part)
    assert [int(v) for v in od.cpu().numpy().view(np.uint64)] == poffs + [2 ** 64 - 1] * 3
    # the host variant
    out = np.full(need + 8, 0x5A, dtype=np.uint8)
    hb = np.array([0, 2000, 2001, n], dtype=np.uint64)
    ho = np.zeros(len(hb), dtype=np.uint64)
    rc = L.slamem_pileup_consensus_host(p._h, 0, n, 4, need, out.ctypes.data, hb.ctypes.data, len(hb), ho.ctypes.data, stats, C.byref(total))
    assert rc == capi.SLAMEM_OK and total.value == need and bytes(out[:need]) == want and bool((out[need:] == 0x5A).all())
    assert [int(v) for v in ho] == cs.consensus(T, t, E, 4, bounds=[0, 2000, 2001, n])[1] and list(stats) == wstats
    out[:] = 0x5A
    rc = L.slamem_pileup_consensus_host(p._h, 0, n, 4, 10, out.ctypes.data, None, 0, None, stats, C.byref(total))
    assert rc == capi.SLAMEM_ERR_CAPACITY and total.value == need and bytes(out[:10]) == want[:10] and bool((out[10:] == 0x5A).all())
    hb[1] = 2501
    rc = L.slamem_pileup_consensus_host(p._h, 2000, 500, 4, need, out.ctypes.data, hb.ctypes.data + 8, 1, ho.ctypes.data, stats, C.byref(total))
    assert rc == capi.SLAMEM_ERR_ARG and b"bound" in L.slamem_last_error_message()
    # refusals
    for bad in (dict(first=n + 1, count=0), dict(first=n - 1, count=2), dict(min_depth=0), dict(min_depth=2 ** 31)):
        with pytest.raises(capi.SlamemError) as err:
            p.consensus(**bad)
        assert err.value.code == capi.SLAMEM_ERR_ARG
    assert L.slamem_pileup_consensus_device(p._h, 0, n, 4, 10, None, None, 0, None, stats, C.byref(total), None) == capi.SLAMEM_ERR_ARG
    assert L.slamem_pileup_consensus_device(p._h, 0, n, 4, 0, None, None, 2, None, stats, C.byref(total), None) == capi.SLAMEM_ERR_ARG
    # nothing of this changed the table or the events
    assert es.from_records(p.events()[0]) == E and np.array_equal(p.counts(), t)
    p.close()
    idx.close()


# ---- real mappings, known answer -----------------------------------------------------------------------------------------------

def sample_case():
    """(reference, sample, reads, offsets): 20 SNVs, a deletion of 3 letters and an insertion of 5, 850 letters apart, placed
    where the letters on both sides rule out any shift; error-free reads of 150 letters at 20x, alternating strands."""
    rng = np.random.default_rng(53)
    n = 20000
    ref = rng.choice(ACGT, size=n)
    sites = [400 + 850 * k for k in range(22)]
    dele, ins = sites[6], sites[15]
    ref[dele - 1:dele + 4] = np.frombuffer(b"ACGTA", dtype=np.uint8)  # rows dele .. dele + 2 (CGT) go: A|CGT|A
    ref[ins - 1:ins + 1] = np.frombuffer(b"AT", dtype=np.uint8)        # GATTC goes between A and T
    pieces, last = [], 0
    for s in sites:
        pieces.append(ref[last:s])
        if s == dele:
            last = s + 3
        elif s == ins:
            pieces.append(np.frombuffer(b"GATTC", dtype=np.uint8))
            last = s
        else:
            pieces.append(ACGT[[(int(np.where(ACGT == ref[s])[0][0]) + 1 + int(rng.integers(0, 3))) % 4]])
            last = s + 1
    pieces.append(ref[last:])
    sample = np.concatenate(pieces)
    assert len(sample) == n + 2
    starts = np.linspace(0, len(sample) - 150, len(sample) * 20 // 150).astype(np.int64)
    reads = [sample[s:s + 150] if k % 2 == 0 else ext_spec.revcomp(sample[s:s + 150]) for k, s in enumerate(starts)]
    q = np.concatenate(reads)
    off = (np.arange(len(reads) + 1, dtype=np.uint64) * np.uint64(150))
    return ref, sample, q, off


def test_real_mappings_give_the_sample_back(eng):
    ref, sample, q, off = sample_case()
    n = len(ref)
    idx = eng.Index.build(ref)
    (qa, oa), (qb, ob) = halves(q, off)
    a, b = eng.Pileup(idx, events=True), eng.Pileup(idx, events=True)
    a.add(qa, oa, 20, True)
    a.add(qb, ob, 20, True)
    b.add(qb, ob, 20, True)
    b.add(qa, oa, 20, True)
    t = a.counts()
    E = es.from_records(a.events()[0])
    assert np.array_equal(b.counts(), t) and es.from_records(b.events()[0]) == E
    want = check(a, bytes(ref), t, E, 4, bounds=[300, n - 300])
    got, offs, stats = b.consensus(4, bounds=[300, n - 300])
    assert bytes(got) == want
    print("statistics", stats, "events", len(E))
    middle = bytes(got[int(offs[0]):int(offs[1])]).upper()
    assert middle == bytes(sample[300:len(sample) - 300])
    assert stats[1] == 20 and stats[2] == 3 and stats[3] == 1 and stats[4] == 5
    for x in (a, b):
        x.close()
    idx.close()


def test_cli_file_is_the_spec_of_the_engines_tables(eng, tmp_path):
    """slaMEM-hip -b -cons ref.fa reads.fa on that data, the reference cut into two records: byte for byte the file cons_spec
    formats from the engine's table and events, and the statistics on stderr."""
    import hostlib
    ref, sample, q, off = sample_case()
    ref = ref.copy()
    ref[10000] = ord("N")
    recs = [ref[:10000], ref[10001:]]
    ref_fa, q_fa = str(tmp_path / "ref.fa"), str(tmp_path / "reads.fa")
    write_fasta(ref_fa, [(b"one first", recs[0]), (b"two\tsecond", recs[1])])
    write_fasta(q_fa, [(b"read%d x" % k, q[int(off[k]):int(off[k + 1])]) for k in range(len(off) - 1)])
    loaded = hostlib.Loaded(ref_fa, 1)
    assert loaded.chars == bytes(ref)
    idx = eng.Index.build(ref)
    p = eng.Pileup(idx, events=True)
    p.add(q, off, 20, True)
    t = p.counts().astype(np.int64)
    E = es.from_records(p.events()[0])
    stats = p.consensus(4)[2]
    p.close()
    idx.close()
    want = cs.fasta_file(t, E, loaded, 4)
    assert want.startswith(b">one\n") and b"\n>two\n" in want and want.count(b">") == 2 and max(len(l) for l in want.split(b"\n")) == 60
    assert want != cs.fasta_file(t, E, loaded, 40)
    base = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    out = str(tmp_path / "cons.fa")
    r = subprocess.run([EXE, "-b", "-cons", "-o", out, ref_fa, q_fa], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=base, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr).decode(errors="replace")[-3000:]
    assert open(out, "rb").read() == want
    line = b"> Consensus: %d positions uncalled, %d called unlike the reference, %d deleted, %d insertions of %d letters\n" % tuple(stats)
    assert line in r.stderr and b"WARNING" not in r.stderr
    assert b"Saving consensus sequences" in r.stdout and b"; minimum depth = 4\n" in r.stdout
    out40 = str(tmp_path / "cons40.fa")
    r = subprocess.run([EXE, "-cons", "-b", "-mdep", "40", "-evs", "4096", "-o", out40, ref_fa, q_fa], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, env=base, timeout=300)
    assert r.returncode == 0 and open(out40, "rb").read() == cs.fasta_file(t, E, loaded, 40)
    for args, message in ((["-cons", "-vcf"], b"Option -cons excludes -mam, -mum, -smem, -chain, -ext, -aln, -paf, -pile, -sites and -vcf"),
                          (["-cons", "-mpct", "20"], b"Option -mpct has no meaning with -cons")):
        r = subprocess.run([EXE] + args + [ref_fa, q_fa], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=base, timeout=60)
        assert r.returncode == 255 and message in r.stdout and b"Building index" not in r.stdout
