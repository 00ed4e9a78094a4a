"""-stats on the MI355X: slamem_stats_*, MapStats, the streams' tables and the executable's report.  Every
comparison is np.array_equal of the whole raw table with tests/stats_spec.py, which walks letter by letter."""
import os
import subprocess

import numpy as np
import pytest

import aln_gap_cases
import aln_spec
import ext_spec
import lowq_spec
import map_spec
import stats_spec
from conftest import search_path
from golden_cases import CASES, MANIFEST, case_paths, opt_value
from test_gpu_aln import batch
from test_gpu_chain import indel_reads
from test_gpu_sam import designed_batch, results_of, seg_ops

pytestmark = pytest.mark.gpu

MEM_CASES = [c for c in CASES if "-mam" not in MANIFEST[c].get("tail", [])]
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "slamem_amd", "host", "slaMEM-hip")
OTHER = {int(a): int(b) for a, b in zip(b"ACGT", b"CGTA")}


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test without a GPU")
    from slamem_amd import engine
    assert engine.STATS_SECTIONS == stats_spec.SECTIONS and engine.STATS_WORDS == stats_spec.WORDS
    return engine


def spec_of(got, ref, q, off, quals=None, min_mapq=0, phred_offset=33):
    return stats_spec.table(results_of(got), bytes(np.asarray(ref, dtype=np.uint8)), q, off, quals, phred_offset, min_mapq)


def one_add(eng, idx, q, off, min_len, both, **kw):
    st = eng.MapStats(idx)
    recs = st.add(q, off, min_len, both, **kw)
    raw = st.raw()
    st.close()
    return raw, recs


def assert_same(got, want):
    for name, (a, n) in stats_spec.SECTIONS.items():
        assert np.array_equal(got[a:a + n], want[a:a + n]), (name, got[a:a + n][:24], want[a:a + n][:24])
    assert np.array_equal(got, want)


@pytest.mark.parametrize("path", ["seed", "walk"])
@pytest.mark.parametrize("case", MEM_CASES)
def test_golden_cases(eng, case, path):
    want_map, _, ref, qs, opts = map_spec.golden_map(case)  # (the spec applied to the file the real reference wrote)
    text = np.frombuffer(ref.chars, dtype=np.uint8).copy()
    idx = eng.Index.build(text)
    q = np.frombuffer(qs.chars, dtype=np.uint8)
    off = np.array(qs.offsets, dtype=np.uint64)
    with search_path(path):
        got, _ = one_add(eng, idx, q, off, int(opt_value(opts, "-l", 20)), "-b" in opts)
    assert_same(got, stats_spec.table(want_map, ref.chars, q, off))
    idx.close()


@pytest.fixture(scope="module")
def constructed(eng):
    """aln_spec.constructed_reads(11) with an unmapped read, a read of no letters and the engine's own mapping of the batch."""
    ref, q, off, _ = aln_spec.constructed_reads(11)
    reads = [q[int(off[i]):int(off[i + 1])] for i in range(len(off) - 1)]
    reads[5:5] = [np.frombuffer(b"N" * 60, dtype=np.uint8).copy(), np.zeros(0, np.uint8)]
    q, off = batch(reads)
    idx = eng.Index.build(ref)
    res = idx.map_reads(q, off, 20, True)
    rng = np.random.default_rng(3)
    quals = (33 + rng.integers(0, 42, size=int(off[-1]))).astype(np.uint8)
    yield dict(ref=ref, q=q, off=off, idx=idx, res=res, quals=quals)
    idx.close()


@pytest.mark.parametrize("min_mapq", [0, 1, 30, 60])
def test_constructed_reads(eng, constructed, min_mapq):
    w = constructed
    got, recs = one_add(eng, w["idx"], w["q"], w["off"], 20, True, min_mapq=min_mapq, quals=w["quals"])
    want = spec_of(w["res"], w["ref"], w["q"], w["off"], w["quals"], min_mapq)
    assert_same(got, want)
    assert np.array_equal(recs, w["res"][4])
    assert want[0] == len(w["off"]) - 1 and want[1] < want[0] and want[88] == 1  # an unmapped read; one of length 0
    if min_mapq == 60:
        assert 0 < want[4] <= want[1]
    st = eng.MapStats(w["idx"])
    st.add_mapped(w["q"], w["off"], w["res"], min_mapq=min_mapq, quals=w["quals"])  # the same from a result the caller has
    assert_same(st.raw(), want)
    tab = st.table()
    assert set(tab) == set(eng.STATS_SECTIONS) and int(tab["totals"][0]) == int(want[0]) and np.array_equal(tab["mapq"], want[24:88])
    st.close()


def test_indel_reads_both_strands_and_empty_batch(eng):
    ref, q, off = indel_reads(21)
    idx = eng.Index.build(ref)
    for both, mq in ((True, 0), (True, 30), (False, 1)):
        got, _ = one_add(eng, idx, q, off, 14, both, min_mapq=mq)
        want = spec_of(idx.map_reads(q, off, 14, both), ref, q, off, None, mq)
        assert_same(got, want)
    assert want[11] > 10 and want[13] > 10  # insertions and deletions
    st = eng.MapStats(idx)
    recs = st.add(q[:0], off[:1], 14, True)  # a batch of 0 reads
    assert len(recs) == 0 and not st.raw().any()
    st.close()
    idx.close()


def long_reads(seed=9):
    """Reads of 510 .. 700 letters on both strands: a substitution at letter 300 (the `=` run behind it crosses cycle 511) and, in
    the reads of 700, one at letter 600 (the run behind it lies wholly behind 511; on strand 2 the run in front of it does); a
    read with an insertion and one with a deletion of 70 letters, and one with both (its edits sum to 127 or more)."""
    rng = np.random.default_rng(seed)
    ref = rng.choice(ACGT, size=30000)
    reads = []
    for k, n in enumerate((510, 511, 512, 513, 700, 700)):
        for rev in (False, True):
            a = 400 + 1500 * len(reads)
            r = ref[a:a + n].copy()
            r[300] = OTHER[int(r[300])]
            if n == 700:
                r[600] = OTHER[int(r[600])]
            reads.append(ext_spec.revcomp(r) if rev else r)
    a = 20000
    ins = np.concatenate([ref[a:a + 120], rng.choice(ACGT, size=70), ref[a + 120:a + 240]])
    dele = np.concatenate([ref[a + 1000:a + 1120], ref[a + 1190:a + 1310]])
    both = np.concatenate([ref[a + 2000:a + 2120], rng.choice(ACGT, size=70), ref[a + 2120:a + 2240], ref[a + 2310:a + 2430]])
    reads += [ins, dele, both, ext_spec.revcomp(ins), ext_spec.revcomp(dele), ext_spec.revcomp(both)]
    q, off = batch(reads)
    return ref, q, off


def test_edges_of_the_walk(eng):
    T = eng.PILE_LANE_OPS
    ref, q, off = designed_batch()  # segments of T - 1, T, T + 1, 63 .. 65, 128 and 129 operations; D directly behind X
    idx = eng.Index.build(ref)
    res = idx.map_reads(q, off, 14, True)
    counts = {len(o) for o in seg_ops(res)}
    assert {T, T + 1, 64, 65, 129} <= counts, sorted(counts)
    assert any(o[i][0] == "X" and o[i + 1][0] == "D" or o[i][0] == "D" and o[i + 1][0] == "X" for o in seg_ops(res) for i in range(len(o) - 1))
    rng = np.random.default_rng(4)
    quals = (33 + rng.integers(0, 42, size=int(off[-1]))).astype(np.uint8)
    for mq in (0, 30):
        got, _ = one_add(eng, idx, q, off, 14, True, min_mapq=mq, quals=quals)
        assert_same(got, spec_of(res, ref, q, off, quals, mq))
    idx.close()
    ref, q, off = long_reads()
    idx = eng.Index.build(ref)
    res = idx.map_reads(q, off, 20, True, max_edits=127)
    want = spec_of(res, ref, q, off)
    a = stats_spec.SECTIONS["cyc_aln"][0]
    assert want[a + 511] > 0 and want[a + 510] > 0 and want[stats_spec.SECTIONS["len"][0] + 511] == 10 and want[88 + 510] == 2
    assert (res[4]["strand"] == 1).sum() >= 6 and (res[4]["strand"] == 2).sum() >= 6
    got, _ = one_add(eng, idx, q, off, 20, True, max_edits=127)
    assert_same(got, want)
    idx.close()
    seen = want.copy()
    # the designed gaps of aln_gap_cases at 127 edits: deletions of up to 127 rows, long insertions, hundreds of operations a segment
    ref, q, off, _ = aln_gap_cases.catalogue()
    idx = eng.Index.build(ref)
    res = idx.map_reads(q, off, aln_gap_cases.MIN_LEN, True, max_edits=127)
    want = spec_of(res, ref, q, off)
    got, _ = one_add(eng, idx, q, off, aln_gap_cases.MIN_LEN, True, max_edits=127)
    assert_same(got, want)
    idx.close()
    seen += want
    nm, il, dl = (int(seen[stats_spec.SECTIONS[s][0] + stats_spec.SECTIONS[s][1] - 1]) for s in ("nm", "ins_len", "del_len"))
    print("reads of 127 edits or more:", nm, "insertions of 63 letters or more:", il, "deletions of 63 or more:", dl)
    assert nm > 0, "a read whose edits sum to 127 or more"
    assert il > 0 and dl > 0


def quality_reads(seed=13):
    """Reads of 400 letters, a substitution every 97 letters, on both strands; the quality bytes run in stretches of 1, 7, 8, 9, 63,
    64 and 65 equal values that start at offsets 0 .. 7 of the read, and hold a byte below the offset, the offset, offset + 93 and
    255."""
    rng = np.random.default_rng(seed)
    ref = rng.choice(ACGT, size=30000)
    reads, quals = [], []
    values = [20, 33, 126, 255, 40, 63, 70, 35]
    for k in range(16):
        a = 300 + 1700 * k
        r = ref[a:a + 400].copy()
        for x in range(50, 400, 97):
            r[x] = OTHER[int(r[x])]
        reads.append(ext_spec.revcomp(r) if k >= 8 else r)
        b, v = [], int(rng.integers(0, 8))
        b += [values[v]] * (k % 8)  # the first long stretch starts at offset k mod 8
        order = list(rng.permutation([1, 7, 8, 9, 63, 64, 65]))
        while len(b) < 400:
            for n in order:
                v = (v + 1 + int(rng.integers(0, 6))) % 8
                b += [values[v]] * int(n)
        quals.append(np.array(b[:400], dtype=np.uint8))
    q, off = batch(reads)
    return ref, q, off, np.concatenate(quals)


def test_qualities(eng):
    ref, q, off, quals = quality_reads()
    assert {20, 33, 126, 255} <= set(int(v) for v in quals)
    idx = eng.Index.build(ref)
    res = idx.map_reads(q, off, 20, True)
    assert (res[4]["strand"] == 1).sum() == 8 and (res[4]["strand"] == 2).sum() == 8
    want = spec_of(res, ref, q, off, quals)
    qa, qm = stats_spec.SECTIONS["q_aln"][0], stats_spec.SECTIONS["q_mm"][0]
    assert want[qa] > 0 and want[qa + 93] > 0 and want[qm:qm + 96].sum() == want[10] > 0
    got, _ = one_add(eng, idx, q, off, 20, True, quals=quals)
    assert_same(got, want)
    import torch
    got, _ = one_add(eng, idx, q, off, 20, True, quals=torch.from_numpy(quals).to(idx.device))  # the bytes as a tensor on the device
    assert_same(got, want)
    got, _ = one_add(eng, idx, q, off, 20, True, quals=quals, phred_offset=64)  # another offset: 20 and 33 clamp to 0
    assert_same(got, spec_of(res, ref, q, off, quals, 0, 64))
    none, _ = one_add(eng, idx, q, off, 20, True)  # quals=None: the two sections stay zero, everything else is equal
    assert not none[qa:qm + 96].any() and np.array_equal(none[:qa], want[:qa]) and np.array_equal(none[qm + 96:], want[qm + 96:])
    st = eng.MapStats(idx)
    with pytest.raises(ValueError):
        st.add(q, off, 20, True, quals=quals, phred_offset=127)
    with pytest.raises(ValueError):
        st.add(q, off, 20, True, min_mapq=61)
    from slamem_amd import capi
    L = capi.lib()
    assert L.slamem_stats_add_device(st._h, None, 1, 0, None, 1, None, 1, 1, None, 127, 0, None) == capi.SLAMEM_ERR_ARG
    assert b"Phred offset" in L.slamem_last_error_message()
    assert L.slamem_stats_add_device(st._h, None, 1, 0, None, 1, None, 1, 1, None, 33, 61, None) == capi.SLAMEM_ERR_ARG
    assert b"mapping quality" in L.slamem_last_error_message() and not st.raw().any()
    st.close()
    idx.close()


@pytest.fixture(scope="module")
def world(eng):
    """150-letter reads with 2 % substitutions on a 100 kbp reference: enough of them that the add's grid has several workgroups and
    one of them walks more reads than it has lanes."""
    n = eng.STATS_BLOCK * (2 * eng.STATS_TRIPS + 2)  # 10 trips: three workgroups of four, three and three trips
    ref = eng.synth_reference(100_000, 42, "cuda:0")
    reads = eng.synth_reads(ref, 0, n, 150, 0.02, 42, 50)[: n * 150].cpu().numpy()
    ref = ref.cpu().numpy()
    off = (np.arange(n + 1, dtype=np.uint64) * np.uint64(150))
    idx = eng.Index.build(ref)
    res = idx.map_reads(reads, off, 20, True)
    rng = np.random.default_rng(8)
    quals = (33 + np.repeat(rng.integers(2, 42, size=(len(reads) + 11) // 12), 12)[:len(reads)]).astype(np.uint8)
    want = spec_of(res, ref, reads, off, quals, 3)
    yield dict(ref=ref, q=reads, off=off, idx=idx, res=res, quals=quals, want=want, n=n)
    idx.close()


def test_more_than_one_workgroup_and_more_than_one_trip(eng, world):
    w = world
    trips = -(-w["n"] // eng.STATS_BLOCK)
    grid = min(-(-trips // eng.STATS_TRIPS), eng.STATS_GRID)
    assert grid >= 3 and trips > grid  # several workgroups, and one of them takes more reads than it has lanes
    got, _ = one_add(eng, w["idx"], w["q"], w["off"], 20, True, min_mapq=3, quals=w["quals"])
    assert_same(got, w["want"])
    assert w["want"][1] > 0.9 * w["n"] and w["want"][3] > 0.3 * w["n"] and w["want"][10] > w["n"]


def test_flush_in_between(eng, world, monkeypatch):
    """SLAMEM_STATS_FLUSH_AT lowers the weight at which a workgroup flushes its LDS table: at 100,000 a flush comes between the
    trips, at 1,000 every trip is heavier than the bound and is walked read by read.  The table is the same."""
    w = world
    for at in ("100000", "1000"):
        monkeypatch.setenv("SLAMEM_STATS_FLUSH_AT", at)
        st = eng.MapStats(w["idx"])
        monkeypatch.delenv("SLAMEM_STATS_FLUSH_AT")
        st.add_mapped(w["q"], w["off"], w["res"], min_mapq=3, quals=w["quals"])
        assert_same(st.raw(), w["want"])
        st.close()


def windows(off, k):
    return [off[a:a + k + 1].copy() for a in range(0, len(off) - 1, k)]


def test_accumulation(eng, world):
    w = world
    half = w["n"] // 2
    st = eng.MapStats(w["idx"])
    st.add(w["q"], w["off"][:half + 1], 20, True, min_mapq=3, quals=w["quals"])
    first = st.raw()
    o2 = w["off"][half:] - w["off"][half]
    st.add(w["q"][int(w["off"][half]):], o2, 20, True, min_mapq=3, quals=w["quals"][int(w["off"][half]):])
    assert_same(st.raw(), w["want"])  # two adds equal one add of the concatenated batch
    st.reset()
    assert not st.raw().any()
    st.add_table(first)
    st.add_table(first)
    assert_same(st.raw(), 2 * first)
    other = eng.MapStats(w["idx"])
    other.add(w["q"][int(w["off"][half]):], o2, 20, True, min_mapq=3, quals=w["quals"][int(w["off"][half]):])
    st.reset()
    st.add_table(first)
    st.add_table(other.raw())
    assert_same(st.raw(), w["want"])
    with pytest.raises(ValueError):
        st.add_table(first[:-1])
    other.close()
    st.close()


def run_stream(eng, w, wins, submit_quals, **kw):
    slots = 3
    st = eng.Stream(w["idx"], slots, 1 << 20, len(wins[0]) - 1, True, min_mapq=3, **kw)

    def submit(b):
        if submit_quals:
            st.submit_quals(w["q"], w["quals"], None, wins[b], 20)
        else:
            st.submit(w["q"], wins[b], 20)
    for b in range(min(slots - 1, len(wins))):
        submit(b)
    for b in range(len(wins)):
        st.next()
        if b + slots - 1 < len(wins):
            submit(b + slots - 1)
    st.close()


def test_streams(eng, world):
    w = world
    wins = windows(w["off"], -(-w["n"] // 3))
    assert len(wins) == 3
    no_quals = w["want"].copy()
    qa, qm = stats_spec.SECTIONS["q_aln"][0], stats_spec.SECTIONS["q_mm"][0]
    no_quals[qa:qm + 96] = 0
    for with_quals in (False, True):
        want = w["want"] if with_quals else no_quals
        t = eng.MapStats(w["idx"])
        run_stream(eng, w, wins, with_quals, paf=True, stats=t, quals=with_quals)
        assert_same(t.raw(), want)
        t.reset()
        p = eng.Pileup(w["idx"])
        run_stream(eng, w, wins, with_quals, pile=p, stats=t, quals=with_quals)
        assert_same(t.raw(), want)
        plain = eng.Pileup(w["idx"])
        run_stream(eng, w, wins, False, pile=plain)
        assert np.array_equal(p.counts(), plain.counts())  # the pile add is untouched
        plain.close()
        p.close()
        t.close()
    # two streams adding into one table give the same as one; a batch through submit on a with_quals stream has no bytes
    t = eng.MapStats(w["idx"])
    run_stream(eng, w, wins[:2], True, paf=True, stats=t, quals=True)
    run_stream(eng, w, wins[2:], True, pile=None, paf=True, stats=t, quals=True)
    assert_same(t.raw(), w["want"])
    t.reset()
    run_stream(eng, w, wins, False, paf=True, stats=t, quals=True)
    assert_same(t.raw(), no_quals)
    t.close()
    # a pile with quality sums and a table: the bytes feed both
    p, t = eng.Pileup(w["idx"], quals=True), eng.MapStats(w["idx"])
    run_stream(eng, w, wins, True, pile=p, stats=t, quals=True)
    assert_same(t.raw(), w["want"])
    assert p.quality.counts().any()
    p.close()
    t.close()


def test_stream_setter_refusals(eng, world):
    import ctypes as C
    import torch
    from slamem_amd import capi
    w = world
    L = capi.lib()
    t = eng.MapStats(w["idx"])
    wins = windows(w["off"], 64)
    st = eng.Stream(w["idx"], 2, 1 << 16, 64, True, paf=True)
    st.submit(w["q"], wins[0], 20)
    assert L.slamem_stream_set_stats(st._h, t._h, 0, 0) == capi.SLAMEM_ERR_ARG  # after a submit
    assert b"before the first submit" in L.slamem_last_error_message()
    st.next()
    st.close()
    assert not t.raw().any()
    for kw in (dict(aln=True), dict()):  # a stream of another match type
        st = eng.Stream(w["idx"], 2, 1 << 16, 64, True, **kw)
        assert L.slamem_stream_set_stats(st._h, t._h, 0, 0) == capi.SLAMEM_ERR_ARG
        assert b"match type 7" in L.slamem_last_error_message()
        st.close()
    st = eng.Stream(w["idx"], 2, 1 << 16, 64, True, paf=True)
    assert L.slamem_stream_set_stats(st._h, t._h, 61, 0) == capi.SLAMEM_ERR_ARG
    assert L.slamem_stream_set_stats(st._h, None, 0, 0) == capi.SLAMEM_ERR_ARG
    assert L.slamem_stream_set_stats(st._h, t._h, 60, 1) == capi.SLAMEM_OK
    st.close()
    with pytest.raises(ValueError):
        eng.Stream(w["idx"], 2, 1 << 16, 64, True, stats=t)
    with pytest.raises(capi.SlamemError):  # submit_quals needs a stream that was told
        st = eng.Stream(w["idx"], 2, 1 << 16, 64, True, paf=True, stats=t)
        try:
            st.submit_quals(w["q"], w["quals"], None, wins[0], 20)
        finally:
            st.close()
    if torch.cuda.device_count() >= 2:  # another device's table
        idx1 = eng.Index.build(w["ref"], "cuda:1")
        t1 = eng.MapStats(idx1)
        st = eng.Stream(w["idx"], 2, 1 << 16, 64, True, paf=True)
        assert L.slamem_stream_set_stats(st._h, t1._h, 0, 0) == capi.SLAMEM_ERR_ARG
        assert b"device" in L.slamem_last_error_message()
        st.close()
        t1.close()
        idx1.close()
    t.close()


def test_compact_index_is_refused(eng):
    from slamem_amd import capi
    ref, q, off, _ = aln_spec.constructed_reads(11, count=8)
    idx = eng.Index.build(ref, layout=capi.LAYOUT_COMPACT)
    assert idx.info.layout == capi.LAYOUT_COMPACT
    st = eng.MapStats(idx)
    empty = (np.zeros(0, eng.ALN_DTYPE), np.zeros(1, np.uint64), np.zeros(0, np.uint32), np.zeros(1, np.uint64), np.zeros(0, eng.MAP_DTYPE))
    with pytest.raises(capi.SlamemError) as e:
        st.add_mapped(q[:0], off[:1], empty)
    assert e.value.code == capi.SLAMEM_ERR_ARG and "text planes" in str(e.value) and "compact" in str(e.value)
    assert "slamem_stats_add_device" in str(e.value)
    s = eng.Stream(idx, 2, 1 << 16, 64, True, mam=False)
    s.close()
    assert not st.raw().any()
    st.close()
    idx.close()


def write_fasta(path, records):
    with open(path, "wb") as fh:
        for name, letters in records:
            fh.write(b">" + name + b"\n")
            for a in range(0, len(letters), 60):
                fh.write(bytes(letters[a:a + 60]) + b"\n")


def run_exe(args, env=None):
    return subprocess.run([EXE] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=300)


def test_executable(eng, tmp_path):
    import torch
    # a golden case (FASTA): the two quality sections stay empty, and stderr says so once
    case = MEM_CASES[0]
    ref_fa, q_fa, _, _ = case_paths(case)
    want_map, _, ref, qs, opts = map_spec.golden_map(case)
    q = np.frombuffer(qs.chars, dtype=np.uint8)
    off = np.array(qs.offsets, dtype=np.uint64)
    want = stats_spec.report(stats_spec.table(want_map, ref.chars, q, off))
    out = str(tmp_path / "golden.stats")
    r = run_exe(list(opts) + ["-stats", "-o", out, ref_fa, q_fa])
    assert r.returncode == 0, (r.stdout + r.stderr).decode(errors="replace")[-3000:]
    assert stats_spec.reports_equal(open(out).read(), want)
    assert r.stderr.count(b"option -stats: FASTA queries carry no base qualities") == 1
    assert b"> Saving mapping statistics to" in r.stdout
    # a small FASTQ written here, with -minq
    ref, q, off, quals = quality_reads(17)
    reads = [q[int(off[i]):int(off[i + 1])] for i in range(len(off) - 1)]
    quals = np.minimum(np.maximum(quals, 33), 126).astype(np.uint8)  # (what a FASTQ file may hold)
    ref_fa, q_fq = str(tmp_path / "ref.fa"), str(tmp_path / "reads.fq")
    write_fasta(ref_fa, [(b"ref one", ref)])
    with open(q_fq, "wb") as fh:
        fh.write(lowq_spec.write_fastq([(b"read%d x" % k, bytes(r), bytes(quals[int(off[k]):int(off[k + 1])])) for k, r in enumerate(reads)]))
    idx = eng.Index.build(ref)
    res = idx.map_reads(q, off, 20, True)
    idx.close()
    want = stats_spec.report(spec_of(res, ref, q, off, quals, 20))
    assert "\nBQ\t" in want and "\nCY\t" in want
    envs = [("one", dict(os.environ))]
    if torch.cuda.device_count() >= 2:
        envs.append(("two", dict(os.environ, SLAMEM_GPUS="2", SLAMEM_BATCH_MB="1", HSA_ENABLE_IPC_MODE_LEGACY="0")))
    for name, env in envs:
        out = str(tmp_path / (name + ".stats"))
        r = run_exe(["-b", "-l", "20", "-stats", "-minq", "20", "-o", out, ref_fa, q_fq], env)
        assert r.returncode == 0, (r.stdout + r.stderr).decode(errors="replace")[-3000:]
        assert stats_spec.reports_equal(open(out).read(), want), name
        assert b"FASTA queries carry no base qualities" not in r.stderr and b"; minimum mapping quality = 20" in r.stdout
    r = run_exe(["-stats", "-paf", ref_fa, q_fq])
    assert r.returncode == 255
    assert b"Option -stats excludes -mam, -mum, -smem, -chain, -ext, -aln, -paf, -sam, -pile, -sites, -vcf, -cons and -depth" in r.stdout + r.stderr


def test_two_gpus_give_the_same_file(eng, tmp_path):
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("one GPU")
    ref, q, off, quals = quality_reads(19)
    reads = [q[int(off[i]):int(off[i + 1])] for i in range(len(off) - 1)]
    ref_fa, q_fa = str(tmp_path / "ref.fa"), str(tmp_path / "reads.fa")
    write_fasta(ref_fa, [(b"ref", ref)])
    write_fasta(q_fa, [(b"read%d" % k, r) for k, r in enumerate(reads)])
    texts = []
    for name, extra in (("one", {}), ("two", dict(SLAMEM_GPUS="2", SLAMEM_BATCH_MB="1", HSA_ENABLE_IPC_MODE_LEGACY="0"))):
        out = str(tmp_path / (name + ".stats"))
        r = run_exe(["-b", "-stats", "-o", out, ref_fa, q_fa], dict(os.environ, **extra))
        assert r.returncode == 0, (r.stdout + r.stderr).decode(errors="replace")[-3000:]
        texts.append(open(out).read())
    assert texts[0] == texts[1]
